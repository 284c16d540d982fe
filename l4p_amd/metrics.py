"""Evaluation metrics on the GPU: the ``metrics_module`` of ``L4PLitModule`` (reference l4p/l4p.py:74-78 calls
``metrics_module(batch, out, metadata) -> (metrics_dict, extras)``; the reference's release carries ``None`` there).

``L4PMetrics`` scores every task whose estimate is in ``out`` and whose ground truth is in ``batch`` with the kernels of
csrc/metrics.hip (definitions at the ``l4p_metric_*`` entries of include/l4p_hip.h, restated in numpy by tests/metrics_restate.py):

  depth     abs_rel, rmse, delta1..3 after a per-clip alignment (median of gt / est, least squares in depth or - "lstsq_inv" - in
            inverse depth, or none); with depth_log_errors=True also sq_rel, rmse_log, log10, silog
  flow      epe, 1px, 3px, 5px
  dyn_mask  iou, precision, recall, f1, accuracy (positive: logit > 0)
  track_2d  the TAP-Vid measures in the 256 x 256 frame: occlusion_accuracy, pts_within_{1,2,4,8,16}, jaccard_{...} and their means
  track_3d  (track_3d="none" | "median" | "track_median" | "query") the same measures on camera-space points: (x, y, z) tracks
            unprojected with the gt intrinsics, the estimate scaled per clip or per track, thresholds that grow with the gt depth
  camray    ate, rpe_trans, rpe_rot (degrees) after a closed-form similarity alignment of the camera centres

Everything stays on the device and nothing synchronises the host: the results are tensors.  A config names the class as
``l4p.metrics.L4PMetrics``.  Not provided: world-frame 3D tracks, TAP-Vid-3D's fixed metric thresholds and windowed scaling,
per-frame alignments.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from .ops import _p, _stream
from .utils.recon4d import _f32

DEPTH_ALIGN = {"none": _lib.L4P_DEPTH_ALIGN_NONE, "median": _lib.L4P_DEPTH_ALIGN_MEDIAN,
               "lstsq": _lib.L4P_DEPTH_ALIGN_LSTSQ}  # the modes of l4p_metric_depth
DEPTH_FULL_ALIGN = {**DEPTH_ALIGN, "lstsq_inv": _lib.L4P_DEPTH_ALIGN_LSTSQ_INV}  # ... of l4p_metric_depth_full
TRACK3D_SCALE = {"none": _lib.L4P_TRACK3D_SCALE_NONE, "median": _lib.L4P_TRACK3D_SCALE_MEDIAN,
                 "track_median": _lib.L4P_TRACK3D_SCALE_TRACK_MEDIAN, "query": _lib.L4P_TRACK3D_SCALE_QUERY}
DENSE_OUT, TRACKS_OUT, CAMERAS_OUT = _lib.L4P_METRIC_DENSE_OUT, _lib.L4P_METRIC_TRACKS_OUT, _lib.L4P_METRIC_CAMERAS_OUT
TRACKS_COUNTS, DEPTH_FULL_OUT = _lib.L4P_METRIC_TRACKS_COUNTS, _lib.L4P_METRIC_DEPTH_FULL_OUT
TAP_THRESHOLDS = (1, 2, 4, 8, 16)
TASKS = ("depth", "flow", "dyn_mask", "track_2d", "camray")

# column of the per-clip result row -> name (after the task prefix); raw sums and counts go to extras only
DEPTH_RAW = {"count": 0, "sum_abs_rel": 1, "sum_sq": 2, "count_delta1": 3, "count_delta2": 4, "count_delta3": 5}
DEPTH_METRICS = {"abs_rel": 6, "rmse": 7, "delta1": 8, "delta2": 9, "delta3": 10}
DEPTH_FULL_RAW = {"sum_sq_rel": 13, "sum_log": 14, "sum_log_sq": 15, "sum_abs_log": 16}  # columns 0..12 as DEPTH_RAW / DEPTH_METRICS
DEPTH_FULL_METRICS = {"sq_rel": 17, "rmse_log": 18, "log10": 19, "silog": 20}
FLOW_RAW = {"count": 0, "sum_epe": 1, "count_1px": 2, "count_3px": 3, "count_5px": 4}
FLOW_METRICS = {"epe": 5, "1px": 6, "3px": 7, "5px": 8}
MASK_RAW = {"tp": 0, "fp": 1, "fn": 2, "tn": 3}
MASK_METRICS = {"iou": 4, "precision": 5, "recall": 6, "f1": 7, "accuracy": 8}
TRACK_RAW = {"count": 0, "count_occ_correct": 1, "count_gt_visible": 2,
             **{f"count_within_{t}": 3 + k for k, t in enumerate(TAP_THRESHOLDS)},
             **{f"count_tp_{t}": 8 + k for k, t in enumerate(TAP_THRESHOLDS)},
             **{f"count_fp_{t}": 13 + k for k, t in enumerate(TAP_THRESHOLDS)}}
TRACK_METRICS = {"occlusion_accuracy": 18, **{f"pts_within_{t}": 19 + k for k, t in enumerate(TAP_THRESHOLDS)},
                 **{f"jaccard_{t}": 24 + k for k, t in enumerate(TAP_THRESHOLDS)}, "average_pts_within_thresh": 29,
                 "average_jaccard": 30}
CAM_RAW = {"align_scale": 3, "sum_sq_ate": 4, "sum_sq_rpe_trans": 5, "sum_sq_rpe_rot": 6, "frames": 7}
CAM_METRICS = {"ate": 0, "rpe_trans": 1, "rpe_rot": 2}


def _u8(x, device) -> torch.Tensor:
    x = torch.as_tensor(x)
    if x.dtype not in (torch.bool, torch.uint8):
        x = x != 0
    return x.to(device=device).contiguous().view(torch.uint8) if x.dtype == torch.bool else x.to(device=device).contiguous()


def _dense(entry: str, est: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor], B: int, n: int, mode: int = 0,
           depth_range: Optional[Tuple[float, float]] = None) -> torch.Tensor:
    lib = _lib.load()
    nbytes = int(lib.l4p_metric_ws_bytes(B, n, mode))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=est.device)
    out = torch.empty(B, DENSE_OUT, dtype=torch.float64, device=est.device)
    if entry == "l4p_metric_depth":
        rc = lib.l4p_metric_depth(_stream(), _p(est), _p(gt), _p(valid), B, n, mode, float(depth_range[0]),
                                  float(depth_range[1]), _p(ws), nbytes, _p(out))
    else:
        rc = getattr(lib, entry)(_stream(), _p(est), _p(gt), _p(valid), B, n, _p(ws), nbytes, _p(out))
    _lib.check(rc, entry)
    return out


def depth_metrics(est, gt, valid=None, align: str = "median", depth_min: float = 1e-3, depth_max: float = 80.0) -> torch.Tensor:
    """[B, 16] float64 rows of ``l4p_metric_depth`` for est, gt (and valid) of shape [B, ...] on the GPU."""
    if align not in DEPTH_ALIGN:
        raise ValueError(f"depth_align is one of {sorted(DEPTH_ALIGN)}, not {align!r}")
    dev = est.device
    est, gt = _f32(est, dev), _f32(gt, dev)
    valid = None if valid is None else _f32(valid, dev)
    B = est.shape[0]
    n = est.numel() // max(B, 1)
    if gt.shape != est.shape or (valid is not None and valid.shape != est.shape):
        raise ValueError(f"depth_metrics: est {tuple(est.shape)}, gt {tuple(gt.shape)} and valid must have one shape")
    return _dense("l4p_metric_depth", est, gt, valid, B, n, DEPTH_ALIGN[align], (depth_min, depth_max))


def depth_metrics_full(est, gt, valid=None, align: str = "median", depth_min: float = 1e-3, depth_max: float = 80.0) -> torch.Tensor:
    """[B, 24] float64 rows of ``l4p_metric_depth_full``: the columns of ``depth_metrics``, then the log-space sums and metrics;
    align may also be "lstsq_inv" (scale and shift in inverse depth)."""
    if align not in DEPTH_FULL_ALIGN:
        raise ValueError(f"depth_align is one of {sorted(DEPTH_FULL_ALIGN)}, not {align!r}")
    dev = est.device
    est, gt = _f32(est, dev), _f32(gt, dev)
    valid = None if valid is None else _f32(valid, dev)
    B = est.shape[0]
    n = est.numel() // max(B, 1)
    if gt.shape != est.shape or (valid is not None and valid.shape != est.shape):
        raise ValueError(f"depth_metrics_full: est {tuple(est.shape)}, gt {tuple(gt.shape)} and valid must have one shape")
    lib, mode = _lib.load(), DEPTH_FULL_ALIGN[align]
    nbytes = int(lib.l4p_metric_depth_full_ws_bytes(B, n, mode))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    out = torch.empty(B, DEPTH_FULL_OUT, dtype=torch.float64, device=dev)
    _lib.check(lib.l4p_metric_depth_full(_stream(), _p(est), _p(gt), _p(valid), B, n, mode, float(depth_min), float(depth_max), _p(ws),
                                         nbytes, _p(out)), "l4p_metric_depth_full")
    return out


def flow_metrics(est, gt, valid=None) -> torch.Tensor:
    """[B, 16] float64 rows of ``l4p_metric_flow`` for est, gt (and valid) of shape [B, 2, ...] on the GPU."""
    dev = est.device
    est, gt = _f32(est, dev), _f32(gt, dev)
    valid = None if valid is None else _f32(valid, dev)
    if est.dim() < 3 or est.shape[1] != 2 or gt.shape != est.shape or (valid is not None and valid.shape != est.shape):
        raise ValueError(f"flow_metrics: est {tuple(est.shape)}, gt {tuple(gt.shape)} and valid must be one shape [B, 2, ...]")
    B = est.shape[0]
    return _dense("l4p_metric_flow", est, gt, valid, B, est.numel() // max(2 * B, 1))


def mask_metrics(logit, gt, valid=None) -> torch.Tensor:
    """[B, 16] float64 rows of ``l4p_metric_mask`` for logit, gt (and valid) of shape [B, ...] on the GPU."""
    dev = logit.device
    logit, gt = _f32(logit, dev), _f32(gt, dev)
    valid = None if valid is None else _f32(valid, dev)
    if gt.shape != logit.shape or (valid is not None and valid.shape != logit.shape):
        raise ValueError(f"mask_metrics: logit {tuple(logit.shape)}, gt {tuple(gt.shape)} and valid must have one shape")
    B = logit.shape[0]
    return _dense("l4p_metric_mask", logit, gt, valid, B, logit.numel() // max(B, 1))


def track_metrics(traj_est, traj_gt, vis_logit, vis_gt, valid, queries, hw: Tuple[int, int]) -> torch.Tensor:
    """[B, 32] float64 rows of ``l4p_metric_tracks``: traj [B, N, 2, T], vis_logit / vis_gt / valid [B, N, (1,) T], queries
    [B, N, 3], hw = (H, W) of the frames the coordinates live in."""
    dev = traj_est.device
    traj_est, traj_gt, queries = _f32(traj_est, dev), _f32(traj_gt, dev), _f32(queries, dev)
    if traj_est.dim() != 4 or traj_est.shape[2] != 2 or traj_gt.shape != traj_est.shape:
        raise ValueError(f"track_metrics: traj_est {tuple(traj_est.shape)} / traj_gt {tuple(traj_gt.shape)}, expected [B, N, 2, T]")
    B, N, _, T = traj_est.shape
    vis_logit = _f32(vis_logit, dev).reshape(B, N, T)
    vis_gt = _u8(vis_gt, dev).reshape(B, N, T)
    valid = None if valid is None else _u8(valid, dev).reshape(B, N, T)
    if tuple(queries.shape) != (B, N, 3):
        raise ValueError(f"track_metrics: queries are {tuple(queries.shape)}, expected [{B}, {N}, 3]")
    counts = torch.empty(B, TRACKS_COUNTS, dtype=torch.int64, device=dev)
    out = torch.empty(B, TRACKS_OUT, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().l4p_metric_tracks(_stream(), _p(traj_est), _p(traj_gt), _p(vis_logit), _p(vis_gt), _p(valid),
                                             _p(queries), B, N, T, int(hw[0]), int(hw[1]), _p(counts), _p(out)),
               "l4p_metric_tracks")
    return out


def track3d_metrics(traj_est, depth_est, traj_gt, depth_gt, vis_logit, vis_gt, valid, queries, intrinsics, hw: Tuple[int, int],
                    scale: str = "median") -> torch.Tensor:
    """[B, 32] float64 rows of ``l4p_metric_tracks3d``: traj [B, N, 2, T], depth_est / depth_gt / vis_logit / vis_gt / valid
    [B, N, (1,) T], queries [B, N, 3], intrinsics [B, 4, 4, T] in the pixel units of the hw = (H, W) frames the tracks live in;
    scale is one of TRACK3D_SCALE."""
    if scale not in TRACK3D_SCALE:
        raise ValueError(f"track_3d scale is one of {sorted(TRACK3D_SCALE)}, not {scale!r}")
    dev = traj_est.device
    traj_est, traj_gt, queries, intrinsics = _f32(traj_est, dev), _f32(traj_gt, dev), _f32(queries, dev), _f32(intrinsics, dev)
    if traj_est.dim() != 4 or traj_est.shape[2] != 2 or traj_gt.shape != traj_est.shape:
        raise ValueError(f"track3d_metrics: traj_est {tuple(traj_est.shape)} / traj_gt {tuple(traj_gt.shape)}, expected [B, N, 2, T]")
    B, N, _, T = traj_est.shape
    if depth_est.numel() != B * N * T or depth_gt.numel() != B * N * T:
        raise ValueError(f"track3d_metrics: depth_est {tuple(depth_est.shape)} / depth_gt {tuple(depth_gt.shape)}, expected "
                         f"[{B}, {N}, (1,) {T}]")
    depth_est, depth_gt = _f32(depth_est, dev).reshape(B, N, T), _f32(depth_gt, dev).reshape(B, N, T)
    vis_logit = _f32(vis_logit, dev).reshape(B, N, T)
    vis_gt = _u8(vis_gt, dev).reshape(B, N, T)
    valid = None if valid is None else _u8(valid, dev).reshape(B, N, T)
    if tuple(queries.shape) != (B, N, 3):
        raise ValueError(f"track3d_metrics: queries are {tuple(queries.shape)}, expected [{B}, {N}, 3]")
    if tuple(intrinsics.shape) != (B, 4, 4, T):
        raise ValueError(f"track3d_metrics: intrinsics are {tuple(intrinsics.shape)}, expected [{B}, 4, 4, {T}]")
    lib, mode = _lib.load(), TRACK3D_SCALE[scale]
    nbytes = int(lib.l4p_metric_tracks3d_ws_bytes(B, N, T, mode))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(B, TRACKS_COUNTS, dtype=torch.int64, device=dev)
    out = torch.empty(B, TRACKS_OUT, dtype=torch.float64, device=dev)
    _lib.check(lib.l4p_metric_tracks3d(_stream(), _p(traj_est), _p(traj_gt), _p(depth_est), _p(depth_gt), _p(vis_logit), _p(vis_gt),
                                       _p(valid), _p(queries), _p(intrinsics), B, N, T, int(hw[0]), int(hw[1]), mode, _p(ws), nbytes,
                                       _p(counts), _p(out)), "l4p_metric_tracks3d")
    return out


def camera_metrics(pose_est, extr_gt) -> torch.Tensor:
    """[B, 8] float64 rows of ``l4p_metric_cameras``: pose_est [B, 16, T] world_T_cam, extr_gt [B, 4, 4, T] cam_T_world."""
    dev = pose_est.device
    pose_est, extr_gt = _f32(pose_est, dev), _f32(extr_gt, dev)
    if pose_est.dim() != 3 or pose_est.shape[1] != 16 or tuple(extr_gt.shape) != (pose_est.shape[0], 4, 4, pose_est.shape[2]):
        raise ValueError(f"camera_metrics: pose_est {tuple(pose_est.shape)} / extr_gt {tuple(extr_gt.shape)}, expected [B, 16, T] "
                         "and [B, 4, 4, T]")
    B, _, T = pose_est.shape
    out = torch.empty(B, CAMERAS_OUT, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().l4p_metric_cameras(_stream(), _p(pose_est), _p(extr_gt), B, T, _p(out)), "l4p_metric_cameras")
    return out


class L4PMetrics(torch.nn.Module):
    """``forward(batch, out, metadata=None) -> (metrics_dict, extras)``.

    A task is scored when its estimate is in ``out`` and its ground truth in ``batch`` (the field names of the reference's L4PData);
    a task with a missing side is skipped.  metrics_dict: 0-d float32 device tensors ``<task>_<metric>``, each the mean over the
    clips of the batch whose value is not NaN (NaN when there is none).  extras: the per-clip float64 tensors [B] under
    ``<task>_<metric>_per_clip``, the raw sums and counts under ``<task>_<name>``, and ``depth_align_scale`` /
    ``depth_align_shift`` [B].

    Opt-in: ``depth_align="lstsq_inv"`` aligns scale and shift in inverse depth; ``depth_log_errors=True`` adds depth_sq_rel,
    depth_rmse_log, depth_log10 and depth_silog; ``track_3d=<scale mode>`` scores ``track_3d_<metric>`` (the names of the 2D
    tracks, plus ``track_3d_scale`` in extras) when the track depths of both sides and ``intrinsics_b44t`` are there and
    ``track_2d`` passes the ``tasks`` filter."""

    def __init__(self, depth_align: str = "median", depth_min: float = 1e-3, depth_max: float = 80.0,
                 tasks: Optional[Sequence[str]] = None, track_3d: Optional[str] = None, depth_log_errors: bool = False):
        super().__init__()
        if depth_align not in DEPTH_FULL_ALIGN:
            raise ValueError(f"depth_align is one of {sorted(DEPTH_FULL_ALIGN)}, not {depth_align!r}")
        if track_3d is not None and track_3d not in TRACK3D_SCALE:
            raise ValueError(f"track_3d is None or one of {sorted(TRACK3D_SCALE)}, not {track_3d!r}")
        if not 0 < depth_min < depth_max:
            raise ValueError(f"need 0 < depth_min < depth_max ({depth_min}, {depth_max})")
        if tasks is not None and set(tasks) - set(TASKS):
            raise ValueError(f"tasks are among {TASKS}, not {sorted(set(tasks) - set(TASKS))}")
        self.depth_align, self.depth_min, self.depth_max = depth_align, float(depth_min), float(depth_max)
        self.tasks = None if tasks is None else tuple(tasks)
        self.track_3d, self.depth_log_errors = track_3d, bool(depth_log_errors)

    @staticmethod
    def _emit(task: str, rows: torch.Tensor, metric_cols: Dict[str, int], raw_cols: Dict[str, int], metrics: dict, extras: dict):
        means = torch.nanmean(rows, dim=0).to(torch.float32)  # per column over the clips that have a value; NaN when none has
        for name, col in metric_cols.items():
            extras[f"{task}_{name}_per_clip"] = rows[:, col]
            metrics[f"{task}_{name}"] = means[col]
        for name, col in raw_cols.items():
            extras[f"{task}_{name}"] = rows[:, col]

    def _wanted(self, task: str, out: dict, batch: dict, est_keys, gt_keys) -> bool:
        return (self.tasks is None or task in self.tasks) and all(k in out for k in est_keys) and all(k in batch for k in gt_keys)

    def _track_hw(self, batch: dict, out: dict) -> Tuple[int, int]:
        for d, k in ((batch, "rgb_b3thw"), (out, "depth_est_b1thw"), (out, "flow_2d_backward_est_b2thw"), (out, "dyn_mask_est_b1thw")):
            if k in d:
                return int(d[k].shape[-2]), int(d[k].shape[-1])
        raise ValueError("L4PMetrics: the track metrics take the frame size from rgb_b3thw in the batch or a dense estimate in out")

    def forward(self, batch: dict, out: dict, metadata=None):
        dev = next((v.device for v in out.values() if torch.is_tensor(v)), None)  # the model's device
        metrics: Dict[str, torch.Tensor] = {}
        extras: Dict[str, torch.Tensor] = {}

        def f32(x):
            return _f32(x, dev)

        if self._wanted("depth", out, batch, ["depth_est_b1thw"], ["depth_b1thw"]):
            valid = batch.get("depth_valid_b1thw")
            full = self.depth_log_errors or self.depth_align == "lstsq_inv"
            rows = (depth_metrics_full if full else depth_metrics)(
                f32(out["depth_est_b1thw"]), f32(batch["depth_b1thw"]), None if valid is None else f32(valid), self.depth_align,
                self.depth_min, self.depth_max)
            self._emit("depth", rows, DEPTH_METRICS, DEPTH_RAW, metrics, extras)
            if self.depth_log_errors:
                self._emit("depth", rows, DEPTH_FULL_METRICS, DEPTH_FULL_RAW, metrics, extras)
            extras["depth_align_scale"], extras["depth_align_shift"] = rows[:, 11], rows[:, 12]
        if self._wanted("flow", out, batch, ["flow_2d_backward_est_b2thw"], ["flow_2d_backward_b2thw"]):
            valid = batch.get("flow_2d_backward_valid_b2thw")
            rows = flow_metrics(f32(out["flow_2d_backward_est_b2thw"]), f32(batch["flow_2d_backward_b2thw"]),
                                None if valid is None else f32(valid))
            self._emit("flow", rows, FLOW_METRICS, FLOW_RAW, metrics, extras)
        if self._wanted("dyn_mask", out, batch, ["dyn_mask_est_b1thw"], ["dyn_mask_b1thw"]):
            valid = batch.get("dyn_mask_valid_b1thw")
            rows = mask_metrics(f32(out["dyn_mask_est_b1thw"]), f32(batch["dyn_mask_b1thw"]), None if valid is None else f32(valid))
            self._emit("dyn_mask", rows, MASK_METRICS, MASK_RAW, metrics, extras)
        if self._wanted("track_2d", out, batch, ["track_2d_traj_est_bn2t", "track_2d_vis_est_bn1t"],
                        ["track_2d_traj_bn2t", "track_2d_vis_bn1t", "track_2d_valid_bn1t", "track_2d_pointquerries_bn3"]):
            H, W = self._track_hw(batch, out)
            rows = track_metrics(f32(out["track_2d_traj_est_bn2t"]), batch["track_2d_traj_bn2t"], out["track_2d_vis_est_bn1t"],
                                 batch["track_2d_vis_bn1t"], batch["track_2d_valid_bn1t"], batch["track_2d_pointquerries_bn3"], (H, W))
            self._emit("track_2d", rows, TRACK_METRICS, TRACK_RAW, metrics, extras)
            if self.track_3d is not None and "track_2d_depth_est_bn1t" in out and "track_2d_depth_bn1t" in batch and \
                    "intrinsics_b44t" in batch:
                rows = track3d_metrics(f32(out["track_2d_traj_est_bn2t"]), out["track_2d_depth_est_bn1t"], batch["track_2d_traj_bn2t"],
                                       batch["track_2d_depth_bn1t"], out["track_2d_vis_est_bn1t"], batch["track_2d_vis_bn1t"],
                                       batch["track_2d_valid_bn1t"], batch["track_2d_pointquerries_bn3"], batch["intrinsics_b44t"],
                                       (H, W), self.track_3d)
                self._emit("track_3d", rows, TRACK_METRICS, TRACK_RAW, metrics, extras)
                extras["track_3d_scale"] = rows[:, 31]
        if self._wanted("camray", out, batch, ["traj3d_est_b16t"], ["extrinsics_b44t"]):
            rows = camera_metrics(f32(out["traj3d_est_b16t"]), batch["extrinsics_b44t"])
            self._emit("camray", rows, CAM_METRICS, CAM_RAW, metrics, extras)
        return metrics, extras
