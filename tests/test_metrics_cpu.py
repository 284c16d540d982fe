"""CPU: the numpy restatement of the evaluation metrics (tests/metrics_restate.py) against hand-checkable identities, the val / test
steps of L4PLitModule with stand-in modules, and the npz -> batch mapping of tools/evaluate.py."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import metrics_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_depth_identities():
    rng = np.random.default_rng(0)
    gt = rng.uniform(0.5, 10.0, 500).astype(F)
    for mode in ("none", "median", "lstsq"):
        r = R.depth(gt, gt, None, mode)
        assert r["count"] == 500 and r["abs_rel"] == 0.0 and r["rmse"] == 0.0
        assert r["delta1"] == r["delta2"] == r["delta3"] == 1.0
    est = (F(2) * gt).astype(F)  # exact in f32: every quotient gt / est is 0.5
    r = R.depth(est, gt, None, "median")
    assert r["align_scale"] == 0.5 and r["align_shift"] == 0.0 and r["abs_rel"] == 0.0 and r["delta1"] == 1.0
    r = R.depth(est, gt, None, "none")
    assert r["abs_rel"] == 1.0 and r["delta1"] == 0.0 and r["delta2"] == 0.0 and r["delta3"] == 0.0  # ratio 2 > 1.953125
    r = R.depth(est, gt, None, "lstsq")
    assert abs(r["align_scale"] - 0.5) < 1e-6 and abs(r["align_shift"]) < 1e-5 and r["abs_rel"] < 1e-6


def test_depth_validity_median_rank_and_empty():
    est = np.asarray([1.0, 2.0, 4.0, 8.0, np.nan, -1.0, 1.0, 1.0], F)
    gt = np.asarray([2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 100.0, np.inf], F)
    valid = np.asarray([1, 1, 1, 1, 1, 1, 1, 1], F)
    assert R.depth_valid(est, gt, valid, 1e-3, 80.0).tolist() == [True] * 4 + [False] * 4
    s, t = R.depth_align(est, gt, valid, "median")  # quotients 2, 1, 0.5, 0.25: the LOWER median of four is rank 1
    assert (float(s), float(t)) == (0.5, 0.0)
    valid[3] = 0  # three left: 2, 1, 0.5 -> rank 1
    assert float(R.depth_align(est, gt, valid, "median")[0]) == 1.0
    valid[:] = 0
    r = R.depth(est, gt, valid, "median")
    assert r["count"] == 0 and all(math.isnan(r[k]) for k in ("abs_rel", "rmse", "delta1", "delta2", "delta3", "align_scale"))
    one = np.asarray([1, 0, 0, 0, 0, 0, 0, 0], F)
    assert math.isnan(R.depth(est, gt, one, "lstsq")["abs_rel"])  # c < 2: no least-squares alignment
    assert R.depth(est, gt, one, "median")["align_scale"] == 2.0


def test_flow_identities():
    rng = np.random.default_rng(1)
    gt = (rng.integers(-40, 40, (2, 300)) / 8.0).astype(F)  # (a grid on which gt + 3 - gt is exactly 3 in f32)
    r = R.flow(gt, gt)
    assert r["count"] == 300 and r["epe"] == 0.0 and r["1px"] == r["3px"] == r["5px"] == 1.0
    est = gt.copy()
    est[0] += F(3)  # epe exactly 3 everywhere: not below 3
    r = R.flow(est, gt)
    assert r["epe"] == 3.0 and r["1px"] == 0.0 and r["3px"] == 0.0 and r["5px"] == 1.0
    valid = np.ones((2, 300), F)
    valid[1, :100] = 0
    gt2 = gt.copy()
    gt2[0, 100:150] = np.nan
    assert R.flow(est, gt2, valid)["count"] == 150
    assert math.isnan(R.flow(est, gt, np.zeros((2, 300), F))["epe"])


def test_mask_known_counts():
    logit = np.asarray([2.0, 0.5, 0.0, -1.0, 3.0, -2.0, 1.0, -0.5], F)  # positive: > 0 (a logit of 0 is negative)
    gt = np.asarray([1.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0], F)
    valid = np.asarray([1, 1, 1, 1, 1, 1, 0, 1], F)
    r = R.mask(logit, gt, valid)
    assert (r["tp"], r["fp"], r["fn"], r["tn"]) == (2, 1, 2, 2)
    assert r["iou"] == 2 / 5 and r["precision"] == 2 / 3 and r["recall"] == 2 / 4 and r["f1"] == 4 / 7 and r["accuracy"] == 4 / 7
    assert math.isnan(R.mask(logit, gt, np.zeros(8, F))["iou"])


def test_tap_two_tracks_four_frames():
    # 256 x 256 frames: distances are pixels.  Track 0 is queried in frame 0, track 1 in frame 1 (frame 0 of it is not valid).
    T = 4
    tg = np.zeros((2, 2, T), F)
    te = np.zeros((2, 2, T), F)
    #            frame:   0     1     2     3
    te[0, 0] = np.asarray([0.0, 0.5, 3.0, 20.0], F)   # track 0: distances 0 (query), 0.5, 3, 20
    te[1, 1] = np.asarray([9.0, 0.0, 1.5, 7.0], F)    # track 1: distances 9 (invalid), 0 (query), 1.5, 7
    vis_gt = np.asarray([[1, 1, 1, 0], [1, 1, 1, 1]], np.uint8)
    logit = np.asarray([[1.0, 1.0, -1.0, 1.0], [1.0, 1.0, 1.0, 1.0]], F)
    valid = np.asarray([[1, 1, 1, 1], [0, 1, 1, 1]], np.uint8)
    q = np.asarray([[0.5, 0, 0], [1.5, 0, 0]], F)
    r = R.tracks(te, tg, logit, vis_gt, valid, q, (256, 256))
    # scored: track 0 frames 1, 2, 3; track 1 frames 2, 3
    assert r["count"] == 5
    # visibility agrees at (0,1), (1,2), (1,3); (0,2) predicted occluded but visible; (0,3) predicted visible but occluded
    assert r["count_occ_correct"] == 3 and r["occlusion_accuracy"] == 3 / 5
    assert r["count_gt_visible"] == 4  # (0,1), (0,2), (1,2), (1,3)
    # distances of the gt-visible frames: 0.5, 3, 1.5, 7
    assert [r[f"count_within_{t}"] for t in (1, 2, 4, 8, 16)] == [1, 2, 3, 4, 4]
    # TP needs predicted visible too: (0,2) drops out
    assert [r[f"count_tp_{t}"] for t in (1, 2, 4, 8, 16)] == [1, 2, 2, 3, 3]
    # FP: predicted visible and not (gt visible and within): (0,3) always; (1,2) at thr 1; (1,3) at thr 1, 2, 4
    assert [r[f"count_fp_{t}"] for t in (1, 2, 4, 8, 16)] == [3, 2, 2, 1, 1]
    assert r["jaccard_1"] == 1 / 7 and r["jaccard_16"] == 3 / 5 and r["pts_within_4"] == 3 / 4
    assert r["average_jaccard"] == pytest.approx((1 / 7 + 2 / 6 + 2 / 6 + 3 / 5 + 3 / 5) / 5, rel=1e-15)
    # est == gt, all visible and predicted visible: AJ = OA = 1
    ones = np.ones((2, T), np.uint8)
    r = R.tracks(tg, tg, np.ones((2, T), F), ones, ones, q, (256, 256))
    assert r["average_jaccard"] == 1.0 and r["occlusion_accuracy"] == 1.0 and r["average_pts_within_thresh"] == 1.0
    # the frame size scales the distance: 3 px in a 128-wide frame are 6 px of the 256 frame
    r = R.tracks(te, tg, logit, vis_gt, valid, q, (256, 128))
    assert [r[f"count_within_{t}"] for t in (1, 2, 4, 8, 16)] == [0, 2, 2, 4, 4]


def test_cameras_exact_similarity_and_reflection():
    T = 12
    Wg = R.make_poses(T, seed=3)
    s, Rm, t = 2.5, R.rot([1.0, 2.0, -0.5], 1.1), np.asarray([3.0, -2.0, 0.7])
    We = Wg.copy()
    We[:, :3, :3] = Rm @ Wg[:, :3, :3]
    We[:, :3, 3] = (s * (Rm @ Wg[:, :3, 3].T)).T + t
    extent = float(np.ptp(Wg[:, :3, 3], axis=0).max())
    # float64 values straight into the float64 stages: the similarity is exact up to rounding
    pose64, extr64 = We.transpose(1, 2, 0).reshape(16, T), np.linalg.inv(Wg).transpose(1, 2, 0)
    r = R.cameras(pose64, extr64, in_dtype=np.float64)
    assert r["ate"] <= 1e-12 * extent and r["rpe_rot"] <= 1e-9 and r["rpe_trans"] <= 1e-12 * extent
    assert abs(r["align_scale"] - 1 / s) < 1e-12
    # through the f32 layout the kernel reads, the rounding of the stored poses bounds the errors instead
    r = R.cameras(pose64.astype(F), extr64.astype(F))
    assert r["ate"] <= 1e-5 * extent and r["rpe_rot"] <= 1e-3 and r["rpe_trans"] <= 1e-5 * extent
    # mirrored centres: the cross-covariance has a negative determinant, the rotation stays proper
    pose_m, extr_m = R.make_camera_case(T, seed=5, reflect=True)
    Pm = pose_m.astype(np.float64).reshape(4, 4, T).transpose(2, 0, 1)
    Gm = np.linalg.inv(extr_m.astype(np.float64).transpose(2, 0, 1))
    s_m, R_m, _, cov = R.umeyama(Pm[:, :3, 3], Gm[:, :3, 3])
    assert np.linalg.det(cov) < 0 and np.linalg.det(R_m) == pytest.approx(1.0, abs=1e-12) and s_m > 0


# ------------------------------------------------------------------------------------------------- L4PLitModule.step
class _StandInModel(torch.nn.Module):
    device = torch.device("cpu")

    def forward(self, batch, tasks):
        return {"depth_est_b1thw": batch["rgb_b3thw"][:, :1] * 2.0, "tasks": list(tasks)}


class _StandInMetrics(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, batch, out, metadata=None):
        self.calls.append((set(batch), set(out), metadata, torch.is_inference_mode_enabled()))
        return {"depth_abs_rel": torch.tensor(0.25, dtype=torch.float64), "flow_epe": torch.tensor(1.5)}, {"depth_count": torch.ones(1)}


class _StandInLoss(torch.nn.Module):
    def forward(self, batch, out):
        return torch.tensor(2.0, dtype=torch.float64), {"l1": torch.tensor(0.5, dtype=torch.float16)}, {"note": 1}


def _module(loss=None, metrics=None):
    from l4p_amd.l4p import L4PLitModule

    return L4PLitModule(["depth"], _StandInModel(), loss_module=loss, metrics_module=metrics)


def test_step_val_and_test_step():
    met = _StandInMetrics()
    m = _module(metrics=met)
    batch = {"rgb_b3thw": torch.ones(1, 3, 2, 4, 4), "seq_name": ["x"]}
    loss, out, skip = m.step("val", batch, 0)
    assert loss == 0 and skip is False and torch.equal(out["depth_est_b1thw"], torch.full((1, 1, 2, 4, 4), 2.0))
    assert set(m.last_log) == {"scalars/val/loss", "scalars/val/depth_abs_rel", "scalars/val/flow_epe"}
    assert m.last_log["scalars/val/loss"] == 0
    for k in ("scalars/val/depth_abs_rel", "scalars/val/flow_epe"):
        assert m.last_log[k].dtype == torch.float32 and m.last_log[k].dim() == 0
    assert float(m.last_log["scalars/val/depth_abs_rel"]) == 0.25
    assert met.calls[-1][2] == {} and met.calls[-1][3] is True  # metadata of the absent loss module; under inference mode
    res = m.test_step(batch, 1)
    assert set(res) == {"loss", "out"} and res["loss"] == 0 and "depth_est_b1thw" in res["out"]
    assert "scalars/val/flow_epe" in m.last_log  # the reference logs its test phase under "val"
    res = m.validation_step(batch, 2)
    assert set(res) == {"loss", "out"}
    loss, out, skip = m.step("test", batch, 0)
    assert "scalars/test/depth_abs_rel" in m.last_log


def test_step_with_loss_module_and_without_metrics():
    m = _module(loss=_StandInLoss())
    batch = {"rgb_b3thw": torch.ones(1, 3, 2, 4, 4)}
    loss, out, skip = m.step("val", batch, 0)
    assert float(loss) == 2.0 and skip is False
    assert set(m.last_log) == {"scalars/val/loss", "scalars/val/l1"}
    assert m.last_log["scalars/val/loss"].dtype == torch.float32 and m.last_log["scalars/val/l1"].dtype == torch.float32
    met = _StandInMetrics()
    m = _module(loss=_StandInLoss(), metrics=met)
    m.step("val", batch, 0)
    assert met.calls[-1][2] == {"note": 1}  # the loss module's metadata reaches the metrics module


def test_step_train_raises_and_predict_unchanged():
    m = _module(metrics=_StandInMetrics())
    batch = {"rgb_b3thw": torch.ones(1, 3, 2, 4, 4)}
    with pytest.raises(NotImplementedError):
        m.step("train", batch, 0)
    out = m.predict_step(batch, 0)
    assert isinstance(out, dict) and torch.equal(out["depth_est_b1thw"], torch.full((1, 1, 2, 4, 4), 2.0))
    assert m.metrics_module.calls == []  # predict scores nothing


def test_metrics_module_is_importable_under_the_alias():
    import l4p.metrics
    import l4p_amd.metrics

    assert l4p.metrics.L4PMetrics is l4p_amd.metrics.L4PMetrics
    with pytest.raises(ValueError):
        l4p_amd.metrics.L4PMetrics(depth_align="log")
    with pytest.raises(ValueError):
        l4p_amd.metrics.L4PMetrics(tasks=["depth", "track_3d"])
    mod = l4p_amd.metrics.L4PMetrics(tasks=["depth"])
    assert mod({"rgb_b3thw": torch.zeros(1, 3, 1, 2, 2)}, {})[0] == {}  # nothing to score: no kernel, no GPU


# ------------------------------------------------------------------------------------------------- tools/evaluate.py
def _evaluate_module():
    spec = importlib.util.spec_from_file_location("l4p_tools_evaluate", os.path.join(ROOT, "tools", "evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_npz_to_batch(tmp_path):
    ev = _evaluate_module()
    T, H, W, N = 3, 4, 5, 2
    clip = {
        "rgb_b3thw": np.zeros((3, T, H, W), np.float64),
        "depth_b1thw": np.ones((1, T, H, W), np.float32),
        "depth_valid_b1thw": np.ones((1, T, H, W), bool),
        "track_2d_traj_bn2t": np.zeros((N, 2, T), np.float32),
        "track_2d_vis_bn1t": np.ones((N, 1, T), bool),
        "track_2d_pointquerries_bn3": np.zeros((N, 3), np.float32),
        "extrinsics_b44t": np.zeros((4, 4, T), np.float32),
        "seq_name": np.asarray("clip0"),
    }
    path = os.path.join(tmp_path, "clip0.npz")
    np.savez(path, **clip)
    with np.load(path) as z:
        batch = ev.npz_to_batch(z)
    assert set(batch) == set(clip)
    assert batch["seq_name"] == ["clip0"]
    assert batch["rgb_b3thw"].shape == (1, 3, T, H, W) and batch["rgb_b3thw"].dtype == torch.float32
    assert batch["depth_valid_b1thw"].shape == (1, 1, T, H, W) and batch["depth_valid_b1thw"].dtype == torch.bool
    assert batch["track_2d_traj_bn2t"].shape == (1, N, 2, T) and batch["track_2d_pointquerries_bn3"].shape == (1, N, 3)
    assert batch["extrinsics_b44t"].shape == (1, 4, 4, T)
    rows = [{"depth_abs_rel": 0.1, "flow_epe": float("nan")}, {"depth_abs_rel": 0.3}]
    mean = ev.mean_over_clips(rows)
    assert mean["depth_abs_rel"] == pytest.approx(0.2) and math.isnan(mean["flow_epe"])
    log = {"scalars/val/loss": 0, "scalars/val/depth_abs_rel": torch.tensor(0.5)}
    assert ev.clip_scalars(log) == {"depth_abs_rel": 0.5}
