"""CPU: the numpy restatement of the 3D-track and full depth metrics (tests/metrics3d_restate.py) against hand-checkable cases,
the properties of the seeded 3D-track cases that the GPU comparison relies on, and the new flags of tools/evaluate.py."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import metrics3d_restate as R3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
THR = (1, 2, 4, 8, 16)


def _axis_case(zg_value=256.0):
    """Two tracks x four frames on the optical axis of a 256 x 256 camera with fx = fy = 256 and the principal point at the origin:
    X = Y = 0, so the 3D distance is |s ze - zg| and the threshold of frame t is thr * zg / 256."""
    T = 4
    K = np.zeros((4, 4, T), F)
    K[0, 0] = K[1, 1] = 256.0
    K[2, 2] = K[3, 3] = 1.0
    traj = np.zeros((2, 2, T), F)
    zg = np.full((2, T), zg_value, F)
    ze = zg.copy()
    #              frame:   0     1     2     3
    ze[0] += np.asarray([0.0, 0.5, 3.0, 20.0], F)  # track 0: distances 0 (query), 0.5, 3, 20
    ze[1] += np.asarray([9.0, 0.0, 1.5, 7.0], F)   # track 1: distances 9 (invalid), 0 (query), 1.5, 7
    vis_gt = np.asarray([[1, 1, 1, 0], [1, 1, 1, 1]], np.uint8)
    logit = np.asarray([[1.0, 1.0, -1.0, 1.0], [1.0, 1.0, 1.0, 1.0]], F)
    valid = np.asarray([[1, 1, 1, 1], [0, 1, 1, 1]], np.uint8)
    q = np.asarray([[0.5, 0, 0], [1.5, 0, 0]], F)
    return dict(traj_est=traj, depth_est=ze, traj_gt=traj, depth_gt=zg, vis_logit=logit, vis_gt=vis_gt, valid=valid, queries=q,
                intrinsics=K, hw=(256, 256))


def test_tracks3d_two_tracks_four_frames():
    c = _axis_case()
    r = R3.tracks3d(**c, scale="none")
    # zg = 256: u = 1, the thresholds are 1, 2, 4, 8, 16 and the case is tests/test_metrics_cpu.py::test_tap_two_tracks_four_frames
    # scored: track 0 frames 1, 2, 3; track 1 frames 2, 3
    assert r["count"] == 5 and r["count_occ_correct"] == 3 and r["count_gt_visible"] == 4
    assert [r[f"count_within_{t}"] for t in THR] == [1, 2, 3, 4, 4]  # gt-visible distances 0.5, 3, 1.5, 7
    assert [r[f"count_tp_{t}"] for t in THR] == [1, 2, 2, 3, 3]
    assert [r[f"count_fp_{t}"] for t in THR] == [3, 2, 2, 1, 1]
    assert r["jaccard_1"] == 1 / 7 and r["pts_within_4"] == 3 / 4 and r["scale"] == 1.0
    # twice the depth: the thresholds double (2, 4, 8, 16, 32) over the same distances
    r = R3.tracks3d(**_axis_case(512.0), scale="none")
    assert [r[f"count_within_{t}"] for t in THR] == [2, 3, 4, 4, 4]
    # a gt depth that is not finite or not positive takes the frame out of the score: (1, 3) with distance 7
    for bad in (np.nan, np.inf, 0.0, -1.0):
        c = _axis_case()
        c["depth_gt"][1, 3] = bad
        r = R3.tracks3d(**c, scale="none")
        assert r["count"] == 4 and r["count_gt_visible"] == 3 and [r[f"count_within_{t}"] for t in THR] == [1, 2, 3, 3, 3]
    # a missing estimate is a miss: (1, 3) stays in the denominators
    c = _axis_case()
    c["depth_est"][1, 3] = np.nan
    r = R3.tracks3d(**c, scale="none")
    assert r["count"] == 5 and r["count_gt_visible"] == 4 and [r[f"count_within_{t}"] for t in THR] == [1, 2, 3, 3, 3]
    assert [r[f"count_fp_{t}"] for t in THR] == [3, 2, 2, 2, 2]  # predicted visible, never within
    # the query scale: zg / ze at the query frame - 1 for track 0; for track 1, with ze halved everywhere, 2 up to the halving of
    # the planted offsets; valid cleared at the query frame leaves no scale
    c = _axis_case()
    c["depth_est"][1] = (c["depth_gt"][1] / F(2)).astype(F)
    r = R3.tracks3d(**c, scale="query")
    assert r["track_scales"].tolist() == [1.0, 2.0] and r["scale"] == 2.0
    assert [r[f"count_within_{t}"] for t in THR] == [3, 3, 4, 4, 4]  # track 1 is exact now: distances 0.5, 3, 0, 0
    c["valid"][1, 1] = 0
    r = R3.tracks3d(**c, scale="query")
    assert math.isnan(r["track_scales"][1]) and r["scale"] == 1.0 and [r[f"count_within_{t}"] for t in THR] == [1, 1, 2, 2, 2]
    assert r["count"] == 5 and r["count_gt_visible"] == 4
    # the lower median: track 0 has the ratios 256 / 256.5, 256 / 259 (eligible: scored and gt visible) -> the smaller one
    c = _axis_case()
    r = R3.tracks3d(**c, scale="track_median")
    assert r["eligible_per_track"].tolist() == [2, 2]
    assert r["track_scales"][0] == F(256) / F(259) and r["track_scales"][1] == F(256) / F(263)
    r = R3.tracks3d(**c, scale="median")  # four ratios 256 / (256.5, 259, 257.5, 263): rank 1 of the sorted ones
    assert r["scale"] == float(F(256) / F(259))


def _scaled_copy(seed=0, B=1, N=12, T=9, hw=(180, 320), hidden=1.7):
    c = R3.make_track3d_case(B, N, T, seed, hw)
    c["traj_est"] = c["traj_gt"].copy()
    zg = np.random.default_rng(seed).uniform(1.0, 8.0, c["depth_gt"].shape).astype(F)
    c["depth_gt"], c["depth_est"] = zg, (zg / F(hidden)).astype(F)
    return c


def test_scale_recovery_and_nan_scale():
    c = _scaled_copy()
    r = R3.tracks3d_of_case(c, 0, "median")
    assert abs(r["scale"] - 1.7) < 1e-6 and r["count_gt_visible"] > 20
    assert r["count_within_1"] == r["count_gt_visible"]  # est = gt / 1.7: the clip's scale brings every frame back
    r0 = R3.tracks3d_of_case(c, 0, "none")
    assert r0["count_within_16"] == 0 and r0["count_gt_visible"] == r["count_gt_visible"]  # and nothing else earns the score
    for mode in ("track_median", "query"):
        rt = R3.tracks3d_of_case(c, 0, mode)
        finite = np.isfinite(rt["track_scales"])
        assert rt["scale"] == finite.sum() and np.all(np.abs(rt["track_scales"][finite] - 1.7) < 1e-6)
    # a track without a scale: its frames are misses, not exclusions
    rt = R3.tracks3d_of_case(c, 0, "track_median")
    assert rt["count_within_1"] == rt["count_gt_visible"]  # (the all-occluded last track has no gt-visible frame to miss)
    c["depth_est"][0, 0] = np.nan  # track 0: no eligible frame any more
    rn = R3.tracks3d_of_case(c, 0, "track_median")
    lost = int((rn["eligible_per_track"] == 0).sum()) - int((rt["eligible_per_track"] == 0).sum())
    assert lost == 1 and math.isnan(rn["track_scales"][0]) and rn["scale"] == rt["scale"] - 1
    assert rn["count"] == rt["count"] and rn["count_gt_visible"] == rt["count_gt_visible"]
    assert rn["count_within_16"] == rt["count_within_16"] - int(rt["eligible_per_track"][0]) < rt["count_within_16"]
    assert rn["pts_within_16"] < 1.0


@pytest.mark.parametrize("B,N,T,hw", [(2, 3, 5, (224, 224)), (1, 70, 24, (180, 320)), (1, 17, 130, (224, 224))])
def test_seeded_cases_reach_what_the_gpu_comparison_needs(B, N, T, hw):
    c = R3.make_track3d_case(B, N, T, seed=7 + N, hw=hw)
    ct = R3.make_track3d_case(B, N, T, seed=7 + N, hw=hw, per_track=True)
    for b in range(B):
        w = R3.tracks3d_of_case(c, b, "median")
        print((B, N, T), "median", [w[f"count_within_{t}"] for t in THR], w["count_gt_visible"], w["scale"])
        if N > 3:
            assert abs(w["scale"] - 1.7) < 0.1
            assert 0 < w["count_within_1"] < w["count_within_2"] < w["count_within_4"] < w["count_within_8"] < w["count_within_16"] \
                < w["count_gt_visible"]
            assert R3.tracks3d_of_case(c, b, "none")["count_within_16"] == 0
        par = set(int(x) % 2 for x in w["eligible_per_track"] if x > 0)
        assert par == {0, 1} or N == 3
        assert (w["eligible_per_track"] == 0).any()
        # the planted pair of frames of track 0: two bit-equal eligible ratios
        assert w["eligible"][0, 1] and w["eligible"][0, 3] and w["ratios"][0, 1] == w["ratios"][0, 3]
        wq = R3.tracks3d_of_case(ct, b, "query")
        print((B, N, T), "query: tracks without a scale", int(np.isnan(wq["track_scales"]).sum()))
        assert np.isnan(wq["track_scales"]).any() and np.isfinite(wq["track_scales"]).any()
        wt = R3.tracks3d_of_case(ct, b, "track_median")
        fin = np.isfinite(wt["track_scales"])
        assert np.all(np.abs(wt["track_scales"][fin] / ct["hidden"][b][fin] - 1.0) < 0.25) and wt["count_within_16"] > 0


def test_depth_full_identities():
    rng = np.random.default_rng(0)
    gt = rng.uniform(0.5, 10.0, 500).astype(F)
    est = (F(2) * gt).astype(F)  # exact in f32
    r = R3.depth_full(est, gt, None, "none")
    assert r["count"] == 500 and r["abs_rel"] == 1.0
    assert r["rmse_log"] == pytest.approx(math.log(2.0), rel=1e-12) and r["log10"] == pytest.approx(math.log10(2.0), rel=1e-12)
    assert r["silog"] < 1e-5  # the variance of a constant, up to the rounding of the two moments
    assert r["sq_rel"] == pytest.approx(float(np.mean(gt.astype(np.float64))), rel=1e-6)  # (gt * gt) / gt
    r = R3.depth_full(est, gt, None, "median")
    assert r["align_scale"] == 0.5 and r["rmse_log"] == 0.0 and r["silog"] == 0.0 and r["sq_rel"] == 0.0
    # an estimate that is affine in inverse depth: 1 / est = 0.5 / gt + 0.1, so 1 / gt = 2 / est - 0.2
    est = (1.0 / (0.5 / gt.astype(np.float64) + 0.1)).astype(F)
    r = R3.depth_full(est, gt, None, "lstsq_inv")
    assert abs(r["align_scale"] - 2.0) < 1e-4 and abs(r["align_shift"] + 0.2) < 1e-4
    assert r["abs_rel"] < 1e-5 and r["rmse_log"] < 1e-5 and r["delta1"] == 1.0 and r["clamped_inv"] == 0
    assert R3.depth_full(est, gt, None, "lstsq")["abs_rel"] > 1e-2  # which a fit in depth does not undo
    # columns shared with the depth entry: the same numbers as its restatement
    from tests import metrics_restate as R

    est = (gt * rng.uniform(0.7, 1.5, 500)).astype(F)
    for mode in ("none", "median", "lstsq"):
        a, b = R.depth(est, gt, None, mode), R3.depth_full(est, gt, None, mode)
        assert all(a[k] == b[k] for k in a)
    # fewer than two elements, or one inverse depth only: no alignment, nothing scored
    one = np.zeros(500, F)
    one[3] = 1
    r = R3.depth_full(est, gt, one, "lstsq_inv")
    assert r["count"] == 0 and all(math.isnan(r[k]) for k in ("abs_rel", "sq_rel", "rmse_log", "log10", "silog", "align_scale"))
    assert R3.depth_full(np.full(500, 2.0, F), gt, None, "lstsq_inv")["count"] == 0


def test_module_arguments_and_evaluate_flags():
    import l4p_amd.metrics as m

    assert m.TRACK3D_SCALE == {"none": 0, "median": 1, "track_median": 2, "query": 3}
    assert set(m.DEPTH_FULL_METRICS) == {"sq_rel", "rmse_log", "log10", "silog"} and max(m.DEPTH_FULL_RAW.values()) == 16
    assert m.TASKS == ("depth", "flow", "dyn_mask", "track_2d", "camray")
    with pytest.raises(ValueError):
        m.L4PMetrics(track_3d="window")
    mod = m.L4PMetrics(track_3d="query", depth_align="lstsq_inv", depth_log_errors=True)
    assert mod({"rgb_b3thw": torch.zeros(1, 3, 1, 2, 2)}, {})[0] == {}  # nothing to score: no kernel, no GPU
    with pytest.raises(ValueError, match="scale"):
        m.track3d_metrics(*([torch.zeros(1, 2, 2, 4)] * 9), (8, 8), scale="window")
    with pytest.raises(ValueError, match="depth_align"):
        m.depth_metrics_full(torch.zeros(1, 8), torch.zeros(1, 8), align="log")
    with pytest.raises(ValueError):
        m.depth_metrics(torch.zeros(1, 8), torch.zeros(1, 8), align="lstsq_inv")  # the 16-column entry keeps its three alignments

    spec = importlib.util.spec_from_file_location("l4p_tools_evaluate3d", os.path.join(ROOT, "tools", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    _, args = ev.parse_args(["DIR", "--synthetic", "--track-3d", "track_median", "--depth-align", "lstsq_inv", "--depth-log-errors"])
    assert (args.track_3d, args.depth_align, args.depth_log_errors) == ("track_median", "lstsq_inv", True)
    _, args = ev.parse_args(["DIR", "--synthetic"])
    assert (args.track_3d, args.depth_align, args.depth_log_errors) == (None, "median", False)
    with pytest.raises(SystemExit):
        ev.parse_args(["DIR", "--synthetic", "--track-3d", "window"])
