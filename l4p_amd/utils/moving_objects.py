"""Moving objects on the GPU (csrc/objects.hip): the motion mask labelled into objects over space-time.

``static_map`` fuses the static pixels of a clip and leaves the movers out; this stage is their side.  The motion mask's foreground
is split into connected components over (t, y, x): neighbours inside a frame, and across frames the pixel the backward flow points
to.  A component's label is its smallest pixel index, kept components are numbered in the order of their first pixel, and every
per-object quantity - pixel counts, boxes, integer coordinate sums, fixed-point sums of the world points - is an integer sum, a
minimum or a maximum: the result is the same bit for bit on every run.  From the labels follow the per-object tables (where each
object is in each frame, in pixels and in the world; how far it moves per frame), the object every point track rides on, and an
overlay video.  The rule, operation by operation, is at ``l4p_objects_label`` in include/l4p_hip.h and in DESIGN.md ("Moving
objects").  The reference has no counterpart: it thresholds the mask for a picture and stops.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream
from . import recon4d

COUNTERS = ("n_pixels", "n_foreground", "n_components", "n_kept", "n_kept_pixels", "n_guard")
MAX_PIXELS = 1 << 30  # labels are 32-bit pixel indices
MAX_ROWS = 1 << 27  # K T rows of the per-object tables
TABLES_2D = ("count", "bbox", "centroid_px")
TABLES_3D = ("count3d", "centroid_xyz", "box3d", "step", "speed")


def _describe(x) -> str:
    return f"{tuple(x.shape)} {x.dtype}" if torch.is_tensor(x) else type(x).__name__


def _check_ids(fn: str, object_id) -> tuple:
    if not torch.is_tensor(object_id) or object_id.dim() != 3 or object_id.dtype != torch.int32 or object_id.numel() < 1:
        raise ValueError(f"{fn}: object_id must be an int32 tensor [T, H, W], got {_describe(object_id)}")
    if object_id.numel() > MAX_PIXELS:
        raise ValueError(f"{fn}: {object_id.numel()} pixels, at most {MAX_PIXELS}")
    return tuple(int(v) for v in object_id.shape)


def _check_label(mask, depth, flow, keep, connectivity, max_depth_ratio, min_pixels, min_frames) -> tuple:
    """Every argument error of ``label_components``, on shapes and host values only: nothing here touches a device."""
    fn = "label_components"
    if not torch.is_tensor(mask) or mask.dim() != 3 or not mask.is_floating_point() or mask.numel() < 1:
        raise ValueError(f"{fn}: mask_thw must be a float tensor [T, H, W] of logits, got {_describe(mask)}")
    T, H, W = (int(v) for v in mask.shape)
    if T * H * W > MAX_PIXELS:
        raise ValueError(f"{fn}: {T * H * W} pixels, at most {MAX_PIXELS}")
    if depth is not None and (not torch.is_tensor(depth) or tuple(depth.shape) != (T, H, W) or not depth.is_floating_point()):
        raise ValueError(f"{fn}: depth_thw must be a float tensor [{T}, {H}, {W}], got {_describe(depth)}")
    if flow is not None and (not torch.is_tensor(flow) or tuple(flow.shape) != (2, T, H, W) or not flow.is_floating_point()):
        raise ValueError(f"{fn}: flow_2thw must be a float tensor [2, {T}, {H}, {W}], got {_describe(flow)}")
    if keep is not None and (not torch.is_tensor(keep) or tuple(keep.shape) != (T, H, W) or keep.dtype not in (torch.uint8, torch.bool)):
        raise ValueError(f"{fn}: keep_thw must be a uint8 or bool tensor [{T}, {H}, {W}], got {_describe(keep)}")
    if connectivity not in (4, 8):
        raise ValueError(f"{fn}: connectivity must be 4 or 8, got {connectivity}")
    r = float(max_depth_ratio)
    if not math.isfinite(r) or (0.0 < r < 1.0):
        raise ValueError(f"{fn}: max_depth_ratio must be finite and <= 0 (no gate) or >= 1, got {max_depth_ratio}")
    if int(min_pixels) < 1:
        raise ValueError(f"{fn}: min_pixels must be >= 1, got {min_pixels}")
    if int(min_frames) < 1:
        raise ValueError(f"{fn}: min_frames must be >= 1, got {min_frames}")
    return T, H, W


def label_components(mask_thw: torch.Tensor, depth_thw: Optional[torch.Tensor] = None, flow_2thw: Optional[torch.Tensor] = None,
                     keep_thw: Optional[torch.Tensor] = None, connectivity: int = 8, max_depth_ratio: float = 0.0, min_pixels: int = 1,
                     min_frames: int = 1) -> Dict[str, object]:
    """Connected components of the motion mask ``mask_thw`` [T, H, W] (logits; foreground is > 0) over space-time.  ``keep_thw``
    (uint8 / bool, 0 = background) and ``depth_thw`` (a pixel without a finite positive depth is background) narrow the foreground;
    inside a frame neighbours (``connectivity`` 4 or 8) are joined where ``max(da, db) <= max_depth_ratio * min(da, db)`` (no gate
    with ``max_depth_ratio`` <= 0 or without depth); across frames a pixel is joined to the pixel of the frame before that
    ``flow_2thw`` [2, T, H, W] (backward flow, channel 0 = x) points to, rounded half up, or to the same pixel without flow.  A
    component is kept with ``min_pixels`` pixels and ``min_frames`` frames.  Returns device tensors, K kept objects in the order of
    their first pixel:

    object_id [T, H, W] int32: the object's number, -1 for background and filtered components;
    label [T, H, W] int32: the smallest pixel index (t H + y) W + x of the pixel's component, -1 for background;
    root, n_pixels, first_frame, last_frame [K] int32 (root = the object's label);
    counters: a host dict of COUNTERS;  K = counters["n_kept"].

    Inputs of any float dtype and layout are converted to contiguous f32 on entry.  The call reads ``counters`` back once (one
    synchronisation) to size the per-object outputs.  ``n_guard`` counts union-find loops that hit their step cap - none can, by
    the argument in csrc/objects.hip; the call raises ``L4PHipError`` if one did."""
    T, H, W = _check_label(mask_thw, depth_thw, flow_2thw, keep_thw, connectivity, max_depth_ratio, min_pixels, min_frames)
    assert mask_thw.is_cuda, "label_components runs on the GPU"
    dev = mask_thw.device
    mask = recon4d._f32(mask_thw, dev)
    depth = recon4d._f32(depth_thw, dev) if depth_thw is not None else None
    flow = recon4d._f32(flow_2thw, dev) if flow_2thw is not None else None
    keep = keep_thw.to(device=dev, dtype=torch.uint8).contiguous() if keep_thw is not None else None
    lib, st = _lib.load(), _stream()
    ws = torch.empty(int(lib.l4p_objects_ws_bytes(T, H, W)), dtype=torch.uint8, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    label, object_id = torch.empty(T, H, W, **i32), torch.empty(T, H, W, **i32)
    counters = torch.empty(len(COUNTERS), dtype=torch.int64, device=dev)
    _lib.check(lib.l4p_objects_label(st, _p(mask), _p(depth), _p(flow), _p(keep), T, H, W, int(connectivity), float(max_depth_ratio),
                                     int(min_pixels), int(min_frames), _p(ws), _p(label), _p(object_id), _p(counters)), "l4p_objects_label")
    host = dict(zip(COUNTERS, (int(v) for v in counters.cpu().tolist())))  # the one host read-back: sizes the outputs
    if host["n_guard"]:
        raise _lib.L4PHipError(f"label_components: {host['n_guard']} union-find loops hit their step cap; the labels are not valid")
    K = host["n_kept"]
    res: Dict[str, object] = {"object_id": object_id, "label": label, "counters": host, "K": K}
    for k in ("root", "n_pixels", "first_frame", "last_frame"):
        res[k] = torch.empty(K, **i32)
    _lib.check(lib.l4p_objects_roots(st, _p(ws), _p(label), _p(object_id), T, H, W, K, _p(res["root"]), _p(res["n_pixels"]),
                                     _p(res["first_frame"]), _p(res["last_frame"])), "l4p_objects_roots")
    return res


def object_tracks(object_id: torch.Tensor, K: int, points: Optional[torch.Tensor] = None,
                  grid: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Where each of the ``K`` objects of ``object_id`` [T, H, W] is in each frame.  From the pixels: count [K, T] int32, bbox
    [K, T, 4] int32 (x0, y0, x1, y1 inclusive; (0, 0, -1, -1) where the object is absent), centroid_px [K, T, 2] f32 (x, y).  With
    ``points`` [T H W, 3] (the world points of ``reconstruct_4d``) and ``grid`` [4] = (ox, oy, oz, v) (``static_map.default_grid``;
    the points are summed in fixed point, steps of v / 256): count3d [K, T] int32, centroid_xyz [K, T, 3], box3d [K, T, 6] (minimum,
    maximum), step [K, T, 3] (centroid of frame t minus that of t - 1; 0 where either is absent) and speed [K, T] = |step|, f32."""
    T, H, W = _check_ids("object_tracks", object_id)
    K = int(K)
    if K < 0 or K * T > MAX_ROWS:
        raise ValueError(f"object_tracks: K must be >= 0 with K T <= {MAX_ROWS}, got K = {K}, T = {T}")
    if (points is None) != (grid is None):
        raise ValueError("object_tracks: points and grid go together")
    if points is not None:
        if not torch.is_tensor(points) or tuple(points.shape) != (T * H * W, 3) or not points.is_floating_point():
            raise ValueError(f"object_tracks: points must be a float tensor [{T * H * W}, 3], got {_describe(points)}")
        if not torch.is_tensor(grid) or grid.numel() != 4 or not grid.is_floating_point():
            raise ValueError("object_tracks: grid must be a float tensor of 4 elements (ox, oy, oz, voxel size)")
    assert object_id.is_cuda, "object_tracks runs on the GPU"
    dev = object_id.device
    ids = object_id.contiguous()
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    res = {"count": torch.empty(K, T, **i32), "bbox": torch.empty(K, T, 4, **i32), "centroid_px": torch.empty(K, T, 2, **f32)}
    pts = g = None
    if points is not None:
        pts, g = recon4d._f32(points, dev), recon4d._f32(grid, dev).reshape(4)
        res.update(count3d=torch.empty(K, T, **i32), centroid_xyz=torch.empty(K, T, 3, **f32), box3d=torch.empty(K, T, 6, **f32),
                   step=torch.empty(K, T, 3, **f32), speed=torch.empty(K, T, **f32))
    if K == 0:  # empty tables, nothing to launch
        return res
    lib = _lib.load()
    ws = torch.empty(int(lib.l4p_objects_tables_ws_bytes(K, T)), dtype=torch.uint8, device=dev)
    _lib.check(lib.l4p_objects_tables(_stream(), _p(ids), _p(pts), _p(g), T, H, W, K, _p(ws), _p(res["count"]), _p(res["bbox"]),
                                      _p(res["centroid_px"]), _p(res.get("count3d")), _p(res.get("centroid_xyz")), _p(res.get("box3d")),
                                      _p(res.get("step")), _p(res.get("speed"))), "l4p_objects_tables")
    return res


def assign_tracks(object_id: torch.Tensor, traj_n2t: torch.Tensor, vis_nt: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The object under every point track: ``traj_n2t`` [N, 2, T] (x, y in pixels of ``object_id``'s grid), ``vis_nt`` [N, T]
    visibility logits.  A track is sampled where its logit is > 0 and its position, rounded half up, lies inside the frame.  Returns
    track_object_nt [N, T] int32 (the id under the track, -1 where it is not sampled or on no object), track_object [N] int32 (the id
    with the most frames, the smallest on a tie, -1 when there is none) and votes [N] int32 (that number of frames)."""
    T, H, W = _check_ids("assign_tracks", object_id)
    if not torch.is_tensor(traj_n2t) or traj_n2t.dim() != 3 or tuple(traj_n2t.shape[1:]) != (2, T) or not traj_n2t.is_floating_point():
        raise ValueError(f"assign_tracks: traj_n2t must be a float tensor [N, 2, {T}], got {_describe(traj_n2t)}")
    N = int(traj_n2t.shape[0])
    if not torch.is_tensor(vis_nt) or tuple(vis_nt.shape) != (N, T) or not vis_nt.is_floating_point():
        raise ValueError(f"assign_tracks: vis_nt must be a float tensor [{N}, {T}], got {_describe(vis_nt)}")
    if N * T > MAX_PIXELS:
        raise ValueError(f"assign_tracks: {N} tracks of {T} frames, at most {MAX_PIXELS} samples")
    assert object_id.is_cuda, "assign_tracks runs on the GPU"
    dev = object_id.device
    i32 = dict(dtype=torch.int32, device=dev)
    res = {"track_object_nt": torch.empty(N, T, **i32), "track_object": torch.empty(N, **i32), "votes": torch.empty(N, **i32)}
    if N == 0:
        return res
    traj, vis = recon4d._f32(traj_n2t, dev), recon4d._f32(vis_nt, dev)
    _lib.check(_lib.load().l4p_objects_tracks(_stream(), _p(object_id.contiguous()), _p(traj), _p(vis), N, T, H, W, _p(res["track_object_nt"]),
                                              _p(res["track_object"]), _p(res["votes"])), "l4p_objects_tracks")
    return res


def object_colours(K: int) -> np.ndarray:
    """uint8 [K, 3]: object k of K in matplotlib's hsv colours, as the track trails are coloured (``recon4d.hsv_index`` /
    ``colour_bytes``)."""
    return recon4d.colour_bytes(recon4d.hsv_table()[recon4d.hsv_index(np.arange(int(K)), int(K))]).reshape(int(K), 3)


def overlay(frames_u8: torch.Tensor, object_id: torch.Tensor, K: int, alpha: int = 128) -> torch.Tensor:
    """``frames_u8`` [T, H, W, 3] uint8 with every object's pixels blended with the object's colour:
    (rgb * (256 - alpha) + colour * alpha + 128) >> 8, ``alpha`` in [0, 256]; other pixels are copied.  Returns a new tensor."""
    T, H, W = _check_ids("overlay", object_id)
    if not torch.is_tensor(frames_u8) or tuple(frames_u8.shape) != (T, H, W, 3) or frames_u8.dtype != torch.uint8:
        raise ValueError(f"overlay: frames_u8 must be a uint8 tensor [{T}, {H}, {W}, 3], got {_describe(frames_u8)}")
    if int(K) < 0:
        raise ValueError(f"overlay: K must be >= 0, got {K}")
    if int(alpha) != alpha or not 0 <= int(alpha) <= 256:
        raise ValueError(f"overlay: alpha must be an integer in [0, 256], got {alpha}")
    assert object_id.is_cuda, "overlay runs on the GPU"
    dev = object_id.device
    frames = frames_u8.to(dev).contiguous()
    lut = torch.from_numpy(object_colours(K)).to(dev) if int(K) > 0 else None
    out = torch.empty_like(frames)
    _lib.check(_lib.load().l4p_objects_overlay(_stream(), _p(frames), _p(object_id.contiguous()), _p(lut), T, H, W, int(K), int(alpha),
                                               _p(out)), "l4p_objects_overlay")
    return out


def moving_objects_from_outputs(batch: dict, out: dict, tasks: List[str], rec: Optional[Dict[str, torch.Tensor]] = None,
                                min_pixels: int = 64, min_frames: int = 2, max_depth_ratio: float = 0.0,
                                connectivity: int = 8) -> Dict[str, object]:
    """``label_components`` and what follows on the engine's outputs.  Needs the dyn_mask task (out["dyn_mask_est_b1thw"]).  Frames
    are linked through out["flow_2d_backward_est_b2thw"] when flow_2d_backward is among the tasks; depth narrows the foreground (and
    gates neighbours with ``max_depth_ratio`` > 0) when depth is; with depth and camray the 3D tables are formed from the world points
    of ``recon4d.reconstruct_4d`` (or the passed ``rec``) on ``static_map.default_grid(out)``; with track_2d every track gets its
    object.  The fields are taken at whatever H x W they have, so the outputs of ``native_res.native_resolution_outputs`` with
    ``native_res.native_batch`` work unchanged.  B = 1 only.  Returns the results of ``label_components``, ``object_tracks`` and
    ``assign_tracks`` in one dict (plus ``grid`` and ``points`` / ``colors`` when the 3D tables were formed).

    The defaults (64 pixels, 2 frames, no depth gate, 8-connectivity) are untuned starting values; no claim rests on them."""
    if "dyn_mask" not in tasks or "dyn_mask_est_b1thw" not in out:
        raise ValueError("moving_objects_from_outputs needs the dyn_mask task and out['dyn_mask_est_b1thw']")
    mask = out["dyn_mask_est_b1thw"]
    if mask.dim() != 5 or mask.shape[1] != 1:
        raise ValueError(f"moving_objects_from_outputs: dyn_mask_est_b1thw must be [1, 1, T, H, W], got {_describe(mask)}")
    assert mask.shape[0] == 1, "Current implementation supports only batch size 1"
    T, H, W = (int(v) for v in mask.shape[2:])
    use_depth = "depth" in tasks and "depth_est_b1thw" in out
    use_flow = "flow_2d_backward" in tasks and "flow_2d_backward_est_b2thw" in out
    res = label_components(mask.reshape(T, H, W), depth_thw=out["depth_est_b1thw"].reshape(T, H, W) if use_depth else None,
                           flow_2thw=out["flow_2d_backward_est_b2thw"].reshape(2, T, H, W) if use_flow else None,
                           connectivity=connectivity, max_depth_ratio=max_depth_ratio, min_pixels=min_pixels, min_frames=min_frames)
    points = grid = None
    if use_depth and "camray" in tasks:
        from . import static_map

        if rec is None:
            rec = recon4d.reconstruct_4d(batch, out, [t for t in tasks if t != "track_2d"])
        points, grid = rec["points"], static_map.default_grid(out)
        res.update(grid=grid, points=points, colors=rec["colors"])
    res.update(object_tracks(res["object_id"], res["K"], points, grid))
    if "track_2d" in tasks and "track_2d_traj_est_bn2t" in out:
        traj, vis = out["track_2d_traj_est_bn2t"], out["track_2d_vis_est_bn1t"]
        res.update(assign_tracks(res["object_id"], traj.reshape(-1, 2, T), vis.reshape(-1, T)))
    return res


def _frames_u8(batch: dict) -> torch.Tensor:
    """The clip as uint8 [T, H, W, 3]: rgb * std + mean, times 255, clamped."""
    rgb = batch["rgb_b3thw"].float()
    dev = rgb.device
    img = rgb * batch["rgb_std_b3111"].to(dev).float() + batch["rgb_mean_b3111"].to(dev).float()
    return (img[0].permute(1, 2, 3, 0) * 255.0).clamp(0, 255).to(torch.uint8).contiguous()


def generate_moving_objects(batch, out, tasks, out_path, res: Optional[Dict[str, object]] = None, **kw) -> str:
    """Writes under ``out_path``: <seq_name>_objects.json (the counters and, per object, its frames, pixels and per-frame bbox,
    centroids and speed), <seq_name>_objects.ply (the world points of the kept objects in their object colours, through
    ``recon4d.write_ply``; only with the 3D tables) and the overlay video <seq_name>_objects (``vis2d.write_video``).  Returns the
    JSON's name."""
    from . import vis2d

    if res is None:
        res = moving_objects_from_outputs(batch, out, tasks, **kw)
    os.makedirs(out_path, exist_ok=True)
    base = os.path.join(out_path, batch["seq_name"][0] + "_objects")
    K = res["K"]
    host = {k: res[k].cpu().numpy() for k in ("root", "n_pixels", "first_frame", "last_frame") + TABLES_2D}
    host.update({k: res[k].cpu().numpy() for k in TABLES_3D if k in res})
    objects = []
    for k in range(K):
        o = dict(id=k, root=int(host["root"][k]), n_pixels=int(host["n_pixels"][k]), first_frame=int(host["first_frame"][k]),
                 last_frame=int(host["last_frame"][k]), count=host["count"][k].tolist(), bbox=host["bbox"][k].tolist(),
                 centroid_px=host["centroid_px"][k].tolist())
        if "speed" in host:
            o.update(count3d=host["count3d"][k].tolist(), centroid_xyz=host["centroid_xyz"][k].tolist(), speed=host["speed"][k].tolist())
        if "track_object" in res:
            o["n_tracks"] = int((res["track_object"] == k).sum())
        objects.append(o)
    with open(base + ".json", "w") as fh:
        json.dump(dict(counters=res["counters"], n_objects=K, objects=objects), fh, indent=1)
    ids = res["object_id"]
    if "points" in res:
        on = torch.nonzero(ids.reshape(-1) >= 0)[:, 0]
        lut = torch.from_numpy(object_colours(K)).to(ids.device) if K else torch.zeros(0, 3, dtype=torch.uint8, device=ids.device)
        recon4d.write_ply(base + ".ply", res["points"][on].cpu().numpy(), lut[ids.reshape(-1)[on].long()].cpu().numpy())
    video = overlay(_frames_u8(batch).to(ids.device), ids, K)
    vis2d.write_video(video.cpu().numpy(), out_path, batch["seq_name"][0] + "_objects")
    return base + ".json"
