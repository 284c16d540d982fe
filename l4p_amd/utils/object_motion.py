"""Object motion and models on the GPU (csrc/object_motion.hip): how every moving object moves, and what it looks like as one body.

``moving_objects`` labels the movers and says where each one is in each frame; an object is still T unrelated per-frame point clouds.
This stage pairs every object pixel with the pixel of the frame before that its backward flow points to (the labelling's own
temporal edges, kept when both ends lie on the same object), fits per object and frame the rigid motion that carries the earlier
points onto the later ones (closed form, from 64-bit integer moments of fixed-point coordinates: the same bit for bit on every run),
refits it on the pairs that agree with the first fit, composes the motions into poses relative to the object's first frame, and
carries every object pixel back into that frame.  There the views of all frames complete one another, and ``static_map.fuse_points``
fuses them into one model per object, as it fuses the background.  The rule, operation by operation, is at ``l4p_objects_motion`` in
include/l4p_hip.h and in DESIGN.md ("Object motion and models").  The reference has no counterpart.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional

import torch

from .. import _lib
from ..ops import _p, _stream
from . import moving_objects, recon4d, static_map

MAX_HW = 1 << 20  # pairs per (object, frame): 2^20 products below 2^42 sum below 2^62
MAX_PIXELS = moving_objects.MAX_PIXELS
MAX_ROWS = moving_objects.MAX_ROWS
TABLES = ("motion", "n_pairs", "n_inliers", "n_far", "rms", "valid", "pose", "pose_valid")
_describe = moving_objects._describe


def _check_motion(object_id, K, points, grid, flow, n_refits, inlier_voxels, min_pairs) -> tuple:
    """Every argument error of ``rigid_motion``, on shapes and host values only: nothing here touches a device."""
    fn = "rigid_motion"
    T, H, W = moving_objects._check_ids(fn, object_id)
    if H * W > MAX_HW:
        raise ValueError(f"{fn}: {H * W} pixels per frame, at most {MAX_HW}")
    if int(K) != K or int(K) < 0 or int(K) * T > MAX_ROWS:
        raise ValueError(f"{fn}: K must be an integer >= 0 with K T <= {MAX_ROWS}, got K = {K}, T = {T}")
    if not torch.is_tensor(points) or tuple(points.shape) != (T * H * W, 3) or not points.is_floating_point():
        raise ValueError(f"{fn}: points must be a float tensor [{T * H * W}, 3], got {_describe(points)}")
    if not torch.is_tensor(grid) or grid.numel() != 4 or not grid.is_floating_point():
        raise ValueError(f"{fn}: grid must be a float tensor of 4 elements (ox, oy, oz, voxel size), got {_describe(grid)}")
    if flow is not None and (not torch.is_tensor(flow) or tuple(flow.shape) != (2, T, H, W) or not flow.is_floating_point()):
        raise ValueError(f"{fn}: flow_2thw must be a float tensor [2, {T}, {H}, {W}], got {_describe(flow)}")
    if int(n_refits) != n_refits or int(n_refits) < 0:
        raise ValueError(f"{fn}: n_refits must be an integer >= 0, got {n_refits}")
    v = float(inlier_voxels)
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{fn}: inlier_voxels must be finite and > 0, got {inlier_voxels}")
    if int(min_pairs) != min_pairs or int(min_pairs) < 3:
        raise ValueError(f"{fn}: min_pairs must be an integer >= 3 (a rotation needs three pairs), got {min_pairs}")
    return T, H, W


def rigid_motion(object_id: torch.Tensor, K: int, points: torch.Tensor, grid: torch.Tensor, flow_2thw: Optional[torch.Tensor] = None,
                 n_refits: int = 1, inlier_voxels: float = 2.0, min_pairs: int = 16, return_moments: bool = False) -> Dict[str, torch.Tensor]:
    """The rigid motion of each of the ``K`` objects of ``object_id`` [T, H, W] (``label_components``) from frame t - 1 to frame t, in
    the world frame of ``points`` [T H W, 3] (``reconstruct_4d``), on ``grid`` [4] = (ox, oy, oz, v) (``static_map.default_grid``; the
    points are summed in fixed point, steps of v / 256).  A pixel is paired with the pixel of the frame before that ``flow_2thw``
    [2, T, H, W] (backward flow, read as ``label_components`` reads it) points to, or with the same pixel without flow, when that
    pixel is on the same object and both points are valid.  The first fit takes every pair; each of the ``n_refits`` refits takes
    the pairs whose residual under the fit before is at most ``inlier_voxels`` voxels.  Returns device tensors:

    motion [K, T, 12] f32: R row-major, then t: p_t ~ R p_(t-1) + t.  Identity and 0 on frame 0, up to the object's first frame and
        without pairs; identity and the step of the pairs' centroid with fewer than ``min_pairs`` inliers;
    n_pairs, n_inliers, n_far [K, T] int32 (n_far: pairs further than 2^21 fixed-point steps from their centre, left out);
    rms [K, T] f32: the RMS residual of the fit over its inliers - the signal that an object does not move rigidly;
    valid [K, T] uint8: n_inliers >= min_pairs;
    pose [K, T, 12] f32: the motions composed from the object's first frame on (identity there and before);
    pose_valid [K, T] uint8: every motion since the first frame was valid;
    canonical [T H W, 3] f32: every object pixel's point carried into the pose of the object's first frame, NaN elsewhere;
    moments [K, T, 18] int64 with ``return_moments``: the integer sums of the last round.

    Inputs of any float dtype and layout are converted to contiguous f32 on entry.  No host read-back.  The defaults (2 voxels, 16
    pairs, one refit) are untuned starting values; no claim rests on them."""
    T, H, W = _check_motion(object_id, K, points, grid, flow_2thw, n_refits, inlier_voxels, min_pairs)
    assert object_id.is_cuda, "rigid_motion runs on the GPU"
    dev, K = object_id.device, int(K)
    ids = object_id.contiguous()
    pts, g = recon4d._f32(points, dev), recon4d._f32(grid, dev).reshape(4)
    flow = recon4d._f32(flow_2thw, dev) if flow_2thw is not None else None
    i32, f32, u8 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev), dict(dtype=torch.uint8, device=dev)
    res = {"motion": torch.empty(K, T, 12, **f32), "n_pairs": torch.empty(K, T, **i32), "n_inliers": torch.empty(K, T, **i32),
           "n_far": torch.empty(K, T, **i32), "rms": torch.empty(K, T, **f32), "valid": torch.empty(K, T, **u8),
           "pose": torch.empty(K, T, 12, **f32), "pose_valid": torch.empty(K, T, **u8),
           "canonical": torch.empty(T * H * W, 3, **f32)}
    if return_moments:
        res["moments"] = torch.empty(K, T, 18, dtype=torch.int64, device=dev)
    if K == 0:  # empty tables, no object pixel, nothing to launch in the library
        res["canonical"].fill_(float("nan"))
        return res
    lib, st = _lib.load(), _stream()
    ws = torch.empty(int(lib.l4p_objects_motion_ws_bytes(K, T)), dtype=torch.uint8, device=dev)
    _lib.check(lib.l4p_objects_motion(st, _p(ids), _p(pts), _p(flow), _p(g), T, H, W, K, int(n_refits), float(inlier_voxels),
                                      int(min_pairs), _p(ws), _p(res["motion"]), _p(res["n_pairs"]), _p(res["n_inliers"]),
                                      _p(res["n_far"]), _p(res["rms"]), _p(res["valid"]), _p(res.get("moments")), _p(res["pose"]),
                                      _p(res["pose_valid"])), "l4p_objects_motion")
    _lib.check(lib.l4p_objects_canonical(st, _p(ids), _p(pts), _p(ws), T, H, W, K, _p(res["canonical"])), "l4p_objects_canonical")
    return res


def object_models(res: Dict[str, object], motion: Dict[str, torch.Tensor], colors: torch.Tensor, T: int,
                  objects: Optional[List[int]] = None, min_frames: int = 2) -> Dict[str, object]:
    """One fused model per object: ``static_map.fuse_points`` on ``motion["canonical"]`` with ``keep = (object_id == k)``, the grid
    ``res["grid"]`` and a table of the smallest power of two >= 2 n_pixels[k] slots, for every object of ``objects`` (default: all
    ``res["K"]``).  ``res`` is the result of ``moving_objects_from_outputs`` (object_id, K, n_pixels, grid), ``colors`` [T H W, 3]
    uint8 the points' colours.  A voxel is kept when ``min_frames`` frames put a point in it.  ``fuse_points`` is used as it is, so
    there is one host read-back (one synchronisation) per object, to size that object's outputs, and one more here for n_pixels.
    Returns ``models`` (a list of the ``fuse_points`` dicts), ``objects`` (their ids) and, concatenated over the objects in that order,
    xyz [V, 3] f32, colors [V, 3] uint8, object [V] int32 and offsets [len(objects) + 1] (host ints: model i is rows
    offsets[i] : offsets[i + 1])."""
    ids, K = res["object_id"], int(res["K"])
    ks = list(range(K)) if objects is None else [int(k) for k in objects]
    if any(k < 0 or k >= K for k in ks):
        raise ValueError(f"object_models: objects must lie in [0, {K}), got {ks}")
    canonical = motion["canonical"]
    dev = canonical.device
    n_pixels = [int(v) for v in res["n_pixels"].cpu().tolist()] if K else []
    models, offsets = [], [0]
    for k in ks:
        m = static_map.fuse_points(canonical, colors, T, grid=res["grid"], keep=(ids == k).reshape(-1), min_frames=min_frames,
                                   table_capacity=static_map.default_capacity(n_pixels[k]))
        models.append(m)
        offsets.append(offsets[-1] + int(m["xyz"].shape[0]))
    cat = lambda key, shape, dt: (torch.cat([m[key] for m in models]) if models else torch.empty(*shape, dtype=dt, device=dev))  # noqa: E731
    obj = [torch.full((offsets[i + 1] - offsets[i],), k, dtype=torch.int32, device=dev) for i, k in enumerate(ks)]
    return {"models": models, "objects": ks, "xyz": cat("xyz", (0, 3), torch.float32), "colors": cat("colors", (0, 3), torch.uint8),
            "object": torch.cat(obj) if obj else torch.empty(0, dtype=torch.int32, device=dev), "offsets": offsets}


def place_models(models: Dict[str, object], pose: torch.Tensor, t: int) -> torch.Tensor:
    """All models of ``object_models`` carried to frame ``t`` by ``pose`` [K, T, 12] (``rigid_motion``), as one cloud [V, 3] f32 in the
    order of ``models["xyz"]`` (colours: ``models["colors"]``)."""
    if not torch.is_tensor(pose) or pose.dim() != 3 or pose.shape[2] != 12 or pose.dtype != torch.float32:
        raise ValueError(f"place_models: pose must be a float32 tensor [K, T, 12], got {_describe(pose)}")
    K, T = int(pose.shape[0]), int(pose.shape[1])
    if int(t) != t or not 0 <= int(t) < max(T, 1):
        raise ValueError(f"place_models: t must be a frame in [0, {T}), got {t}")
    xyz, obj = models["xyz"].contiguous(), models["object"].contiguous()
    out = torch.empty_like(xyz)
    if xyz.shape[0] == 0:
        return out
    assert xyz.is_cuda, "place_models runs on the GPU"
    _lib.check(_lib.load().l4p_objects_place(_stream(), _p(xyz), _p(obj), _p(pose.contiguous()), int(xyz.shape[0]), K, T, int(t), _p(out)),
               "l4p_objects_place")
    return out


def object_motion_from_outputs(batch: dict, out: dict, tasks: List[str], res: Optional[Dict[str, object]] = None,
                               rec: Optional[Dict[str, torch.Tensor]] = None, n_refits: int = 1, inlier_voxels: float = 2.0,
                               min_pairs: int = 16, min_frames: int = 2, **kw) -> Dict[str, object]:
    """``rigid_motion`` and ``object_models`` on the engine's outputs.  ``res`` is the result of
    ``moving_objects.moving_objects_from_outputs``, which is run (with ``rec`` and ``**kw``) when it is not given; it needs the
    dyn_mask, depth and camray tasks (the 3D tables), and the pairs follow out["flow_2d_backward_est_b2thw"] when flow_2d_backward
    is among the tasks.  The fields are taken at whatever H x W they have, so the outputs of
    ``native_res.native_resolution_outputs`` with ``native_res.native_batch`` work unchanged.  B = 1 only.  Returns ``res`` with
    ``motion`` (the dict of ``rigid_motion``) and ``models`` (the dict of ``object_models``) added."""
    if res is None:
        res = moving_objects.moving_objects_from_outputs(batch, out, tasks, rec=rec, **kw)
    if "points" not in res:
        raise ValueError("object_motion_from_outputs needs the world points: the dyn_mask, depth and camray tasks")
    ids = res["object_id"]
    T, H, W = (int(v) for v in ids.shape)
    use_flow = "flow_2d_backward" in tasks and "flow_2d_backward_est_b2thw" in out
    flow = out["flow_2d_backward_est_b2thw"].reshape(2, T, H, W) if use_flow else None
    res = dict(res)
    res["motion"] = rigid_motion(ids, res["K"], res["points"], res["grid"], flow, n_refits=n_refits, inlier_voxels=inlier_voxels,
                                 min_pairs=min_pairs)
    res["models"] = object_models(res, res["motion"], res["colors"], T, min_frames=min_frames)
    return res


def generate_object_models(batch, out, tasks, out_path, res: Optional[Dict[str, object]] = None, **kw) -> str:
    """Writes under ``out_path``: <seq_name>_object_models.ply (every object's fused model at the pose of its first frame, in its true
    colours, through ``recon4d.write_ply``) and <seq_name>_object_motion.json (per object and frame motion, pose, valid, pose_valid,
    n_pairs, n_inliers, n_far and rms; per model the counters of its fusion and compression = n_used / n_kept, null for an empty
    model).  ``res``: the result of ``object_motion_from_outputs``, run with ``**kw`` when not given.  Returns the JSON's name."""
    if res is None or "models" not in res:
        res = object_motion_from_outputs(batch, out, tasks, res=res, **kw)
    os.makedirs(out_path, exist_ok=True)
    seq = batch["seq_name"][0]
    mo, md = res["motion"], res["models"]
    recon4d.write_ply(os.path.join(out_path, seq + "_object_models.ply"), md["xyz"].cpu().numpy(), md["colors"].cpu().numpy())
    host = {k: mo[k].cpu().numpy() for k in TABLES}
    first = res["first_frame"].cpu().tolist()
    objects = []
    for i, k in enumerate(md["objects"]):
        c = md["models"][i]["counters"]
        o = dict(id=k, first_frame=int(first[k]), n_vertices=md["offsets"][i + 1] - md["offsets"][i], counters=c,
                 compression=c["n_used"] / c["n_kept"] if c["n_kept"] else None)
        o.update({key: host[key][k].tolist() for key in TABLES})
        objects.append(o)
    name = os.path.join(out_path, seq + "_object_motion.json")
    with open(name, "w") as fh:
        json.dump(dict(n_objects=int(res["K"]), n_vertices=md["offsets"][-1], voxel_size=float(res["grid"][3]), objects=objects), fh, indent=1)
    return name
